"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan_var on device rows (one observed scan plus P
permutations in one call) against cnf2_qtl_scan_binary at the same shape on the same rows, with the mean iterations per fit
of the observed column, the share of the fits by status, and the device's clock.  One process, the calls alternating, on a
synthetic F2 (synth.make_f2): by default 1 000 individuals x 10 chromosomes x 499 SNPs (+1 dummy marker each) = 5 000
markers, one trait with a mean locus and a variance locus, two covariates of which one is a variance covariate, 100
permutations, tol = 1e-7 and max_iter = 50 for both scans; the binary scan takes the trait's sign.
usage: python tools/qtlvar_timing.py [individuals=1000] [snps_per_chrom=499] [chroms=10] [repeats=3] [P=100]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

a = [int(x) for x in sys.argv[1:6]] + [1000, 499, 10, 3, 100][len(sys.argv[1:6]):]
n, snps, chroms, reps, P = a
ped = synth.make_f2(n, snps, chroms, seed=2)
ctx = capi.Context(0)
ctx.upload(ped)
M = ped.n_markers
org = qtl.origin_rows(ctx)
m1, m2 = M // 3, (2 * M) // 3
g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
z = np.stack([np.where(synth.uniform(78, np.arange(n)) < 0.5, -0.5, 0.5), synth.uniform(79, np.arange(n)) - 0.5], axis=1)
u1, u2 = synth.uniform(77, np.arange(n)), synth.uniform(76, np.arange(n))
e = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
y = (0.3 * g(m1) + 0.8 * z[:, 0] + np.exp(0.5 * (0.4 * g(m2) + 0.5 * z[:, 0])) * e)[:, None]
b = (y > np.median(y)).astype(np.float64)
perm = qtl.permutations(n, P, 3) if P else None
out = {}


def scan_var():
    out["var"] = ctx.qtl_scan_var_device(n, org.data_ptr(), y, cov=z, n_var=1, perm=perm, max_iter=50, tol=1e-7)     # (ends in the call's own synchronise)


def scan_binary():
    out["bin"] = ctx.qtl_scan_binary_device(n, org.data_ptr(), b, cov=z, perm=perm, max_iter=50, tol=1e-7)


calls = [("cnf2_qtl_scan_var", scan_var), ("cnf2_qtl_scan_binary", scan_binary)]
for _, fn in calls:
    fn()
times = {name: [] for name, _ in calls}
for _ in range(reps):
    for name, fn in calls:
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
prop = torch.cuda.get_device_properties(0)
try:
    clock = "%d MHz" % torch.cuda.clock_rate(0)         # the shader clock as the management library reports it now
except Exception as e:                                  # (no management library: the clock is not known, and that is said)
    clock = "not reported (%s)" % type(e).__name__
print("%s (%s), %d compute units, clock %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, clock))
print("%d F2 x %d markers (%d chromosomes), one trait, two covariates (one in the variance part), 1 + %d columns, best of %d; times in s, "
      "ending in a synchronise" % (n, M, chroms, P, reps))
for name, _ in calls:
    print("  %-22s %.4f (all: %s)" % (name, min(times[name]), " ".join("%.4f" % v for v in times[name])))
o = out["var"]
fitted = o["rank"] > 0
for k, name in enumerate(("mean-only", "variance-only", "full")):
    it, st = o["iters"][0][fitted, k], o["status"][0][fitted, k]
    print("  variance scan, %s fit of the observed column: mean iterations %.2f, largest %d; status 0 / 1 / 2 at %.4f / %.4f / %.4f of the fits" %
          (name, it.mean(), it.max(), (st == 0).mean(), (st == 1).mean(), (st == 2).mean()))
for k, (name, at) in enumerate((("joint", m1), ("mean", m1), ("variance", m2))):
    print("  %s LOD: peak %.2f at marker %d (planted %d)" % (name, o["lod"][0, :, k].max(), int(o["lod"][0, :, k].argmax()), at))
ob = out["bin"]
fb = ob["rank"] > 0
print("  binary scan (of the trait's sign), observed column: mean iterations per fit %.2f, largest %d" % (ob["iters"][0][fb].mean(), ob["iters"][0][fb].max()))
tv, tb = (min(times[name]) for name, _ in calls)
# a fit of t iterations without a halving walks the individuals 2 t + 1 times; the permuted columns' counts are not reported,
# so the observed column's mean stands for all of them
passes = float((2 * o["iters"][0][fitted] + 1).sum()) * (1 + P)
print("  scan_var / scan_binary %.2f; about %.3g passes x %d individuals in the variance scan: %.3g individual-passes per second" %
      (tv / tb, passes, n, passes * n / tv))
if P:
    th = qtl.thresholds_var(o["perm_max"])
    print("  5 %% genome-wide thresholds: joint %.2f, mean %.2f, variance %.2f" % tuple(th[k]["genome"][0, 0] for k in qtl.VAR_KEYS))
ctx.close()
