"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan_em on device rows against cnf2_qtl_scan on the
same rows and against the origin sweep that makes the rows (cnf2_sweep_origins, device outputs); the histogram of the fits'
iteration counts and the share that stopped at max_iter; bytes and FP64 operations per fit-iteration, counted from the code
(cnf2_qtlem.h, cnf2_qtlem_kernels.hip), against the MI355X's peaks.  One process, the calls alternating, on a synthetic F2
(synth.make_f2); config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker each), one trait, one
covariate, P permutations for every P of the list, tol = 1e-6, max_iter = 1000.
usage: python tools/qtlem_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3] [P,P,...=0,10]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

HBM, PEAK = 8.0e12, 78.6e12          # bytes/s and f64 FLOP/s of the MI355X
TOL, MAX_ITER = 1e-6, 1000
a = [int(x) for x in sys.argv[1:5]] + [10000, 2500, 20, 3][len(sys.argv[1:5]):]
n, snps, chroms, reps = a
perms = [int(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "0,10").split(",")]
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
m1 = M // 3
g = ped.allele[3:, m1, :].astype(np.float64).sum(axis=1) - 3.0
z = np.where(synth.uniform(78, np.arange(n)) < 0.5, -0.5, 0.5)[:, None]
pheno = (0.3 * g + 0.4 * z[:, 0] + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
K = 1
# One individual in one pass of one fit (qtlem_terms, no imprinting): it reads its 32-byte origin row, 8 bytes of the
# column image, 8 K bytes of covariates and a mask byte; counted as FP64 operations (an FMA as two, exp and log by the
# ~25 and ~30 the device library's polynomial and reconstruction take, a division as ~10): the prior 3 + 4 x 10, the mean
# 2 (K + 1), three residuals and exponents 12, the maximum 3, three exp 75 and their products 3, the sum and log 2 + 30 + 1,
# the weights 10 + 3, e_bar 2, the sums 2 x 3 (K + 1) + 2 x 3 + 4.
BYTES = 32 + 8 + 8 * K + 1
FLOPS = (3 + 40) + 2 * (K + 1) + 12 + 3 + 75 + 3 + 33 + 13 + 2 + 6 * (K + 1) + 6 + 4
print("%d F2 x %d markers (%d chromosomes; input %.1f s), one trait, one covariate, best of %d; times in s, ending in a synchronise; "
      "tol %g, max_iter %d" % (n, M, chroms, gen_s, reps, TOL, MAX_ITER))
for P in perms:
    R = 1 + P
    perm = qtl.permutations(n, P, 3) if P else None
    res = qtl.null_residuals(pheno, z)
    out = {}

    def scan():
        out["scan"] = ctx.qtl_scan_device(n, org.data_ptr(), res, cov=z, perm=perm)          # (ends in the call's own synchronise)

    def scan_em():
        out["em"] = ctx.qtl_scan_em_device(n, org.data_ptr(), res, cov=z, perm=perm, max_iter=MAX_ITER, tol=TOL)

    calls = [("cnf2_sweep_origins", sweep), ("cnf2_qtl_scan", scan), ("cnf2_qtl_scan_em", scan_em)]
    for _, fn in calls:
        fn()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    tw, ts, te = (min(times[name]) for name, _ in calls)
    print("P = %d (R = %d columns)" % (P, R))
    for name, _ in calls:
        print("  %-20s %.4f (all: %s)" % (name, min(times[name]), " ".join("%.4f" % v for v in times[name])))
    em, one = out["em"], out["scan"]
    it = em["iters"][0]
    fitted = em["rank"] > 0
    edges = [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513, MAX_ITER + 1]
    hist = np.histogram(it, bins=edges)[0]
    print("  scan_em / scan %.1f, scan_em / sweep %.2f" % (te / ts, te / tw))
    print("  observed column: %d of %d markers fitted; iters " % (fitted.sum(), M) +
          ", ".join("%d..%d: %d" % (edges[k], edges[k + 1] - 1, hist[k]) for k in range(len(hist)) if hist[k]) +
          "; mean %.2f, largest %d; status 1 at %.4f of the fits, status 2 at %.4f" %
          (it[fitted].mean() if fitted.any() else 0.0, it.max(), (em["status"][0][fitted] == 1).mean() if fitted.any() else 0.0,
           (em["status"][0][fitted] == 2).mean() if fitted.any() else 0.0))
    # every fit of t iterations walks the individuals t + 1 times; the permuted columns' counts are not reported, so the
    # observed column's mean stands for all of them
    passes = float((it[fitted] + 1).sum()) * R
    print("  per fit-iteration %d bytes and %d FP64 operations per individual: about %.3g passes x %d individuals = %.3g B and %.3g FLOP; "
          "at the measured time %.2f TB/s = %.3f of the %.0f TB/s HBM peak (were every row read from HBM), %.2f TFLOP/s = %.3f of the %.1f "
          "TFLOP/s f64 peak" % (BYTES, FLOPS, passes, n, passes * n * BYTES, passes * n * FLOPS, passes * n * BYTES / te / 1e12,
                                passes * n * BYTES / te / HBM, HBM / 1e12, passes * n * FLOPS / te / 1e12, passes * n * FLOPS / te / PEAK,
                                PEAK / 1e12))
    print("  largest |lod_em - lod_hk| %.3f; EM peak %.2f at marker %d, HK peak %.2f at marker %d (planted %d)%s" % (
        np.abs(em["lod"] - one["lod"]).max(), em["lod"][0].max(), int(em["lod"][0].argmax()), one["lod"][0].max(),
        int(one["lod"][0].argmax()), m1,
        "; 5 %% genome-wide thresholds EM %.2f, HK %.2f" % (qtl.thresholds(em["perm_max"])["genome"][0, 0],
                                                          qtl.thresholds(one["perm_max"])["genome"][0, 0]) if P else ""))
ctx.close()
