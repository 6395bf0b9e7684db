"""Measurement aid: wall time, ending in the call's own synchronise, of cnf2_qtl_scan_fam beside cnf2_qtl_scan (additive) on the
same device rows and the same columns, in one process, the two alternating, best of `repeats`.  Config 2's shape: n
individuals x `chroms` chromosomes of `snps` + 1 markers, as `families` families of n / families members (one cell each), K
covariates, one trait and P permutations drawn inside the families.  The rows are soft one-hot rows made on the device
(neither scan looks at where its rows come from); the two products are the same number of multiply-adds, n x M x R, and the
within-family scan adds a fold of about (K + 2) operations per (family, marker, column) and reads the design kernel's records.
usage: python tools/qtlfam_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [families=500] [K=2] [P=255] [repeats=3]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

PEAK = 78.6e12          # f64 matrix peak of the MI355X, FLOP/s
a = [int(x) for x in sys.argv[1:8]] + [10000, 2500, 20, 500, 2, 255, 3][len(sys.argv[1:8]):]
n, snps, chroms, F, K, P, reps = a
M, dev = chroms * (snps + 1), torch.device("cuda", 0)
cs = np.arange(chroms + 1, dtype=np.int32) * (snps + 1)
ctx = capi.Context(0)
ctx.upload_map(np.tile(np.arange(snps + 1, dtype=np.float64) * 0.04, chroms), cs)
gen = torch.Generator(device=dev)
gen.manual_seed(5)
org = torch.empty((n, M, 4), dtype=torch.float64, device=dev)
for i0 in range(0, n, 500):                     # (in slabs: the generator's temporaries stay small beside the 16 GB of rows)
    r = torch.rand((min(500, n - i0), M, 4), dtype=torch.float64, device=dev, generator=gen) ** 8
    org[i0:i0 + r.shape[0]] = r / r.sum(dim=2, keepdim=True)
torch.cuda.synchronize(dev)
grp = (np.arange(n) * F // n).astype(np.int32)
x = (org[:, M // 3, 1] + org[:, M // 3, 3] - org[:, M // 3, 0] - org[:, M // 3, 2]).cpu().numpy()
cov = synth.uniform(9, np.arange(n * K)).reshape(n, K) * 2.0 - 1.0 if K else None
pheno = (np.where(grp % 2 == 0, 0.3, -0.3) * x + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
res = qtl.cell_residuals(pheno, grp, cov)
perm = qtl.permutations(n, P, 3, strata=grp) if P else None
R = 1 + P
print("%d individuals in %d families x %d markers (%d chromosomes), K = %d, one trait, P = %d (R = %d columns), best of %d; times in s, "
      "ending in the call's synchronise" % (n, F, M, chroms, K, P, R, reps), flush=True)
out = {}


def line():
    out["line"] = ctx.qtl_scan_device(n, org.data_ptr(), res, cov=cov, perm=perm, additive=True)


def fam():
    out["fam"] = ctx.qtl_scan_fam_device(n, org.data_ptr(), 0, grp, F, res, cov=cov, perm=perm)


calls = [("cnf2_qtl_scan (additive)", line), ("cnf2_qtl_scan_fam", fam)]
for _, fn in calls:             # warm: code objects, the context's buffers
    fn()
clock0 = ctx.clock_probe()
times = {name: [] for name, _ in calls}
for _ in range(reps):
    for name, fn in calls:
        t1 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t1)
clock1 = ctx.clock_probe()
best = {k: min(v) for k, v in times.items()}
flop = 2.0 * n * M * R
for name, _ in calls:
    print("  %-26s best %.4f (all: %s)  %.2f TFLOP/s of the product (%.3f of the f64 matrix peak)" % (
        name, best[name], " ".join("%.4f" % v for v in times[name]), flop / best[name] / 1e12, flop / best[name] / PEAK))
fold = float(F) * M * R * (K + 2)
print("  cnf2_qtl_scan_fam takes %.2f x cnf2_qtl_scan (additive): the same %.3g multiply-adds; the fold adds %.3g operations "
      "(%.4f of them) on the vector units, and the records read are %.0f MB ((1 + K) doubles per family and marker)" % (
          best["cnf2_qtl_scan_fam"] / best["cnf2_qtl_scan (additive)"], flop / 2, fold, fold / (flop / 2), F * M * (1 + K) * 8 / 1e6))
print("  shader clock %.0f MHz before, %.0f MHz after" % (clock0, clock1))
g, l = out["fam"], out["line"]
top = int(np.argmax(g["lod"][0]))
thr = qtl.thresholds(g["perm_max"])["genome"][0, 0] if P else float("nan")
print("  within-family peak %.2f at marker %d (planted %d), df %d, 5 %% threshold %.2f; line-cross LOD there %.2f" % (
    g["lod"][0, top], top, M // 3, g["df"][top], thr, l["lod"][0, M // 3]))
ctx.close()
