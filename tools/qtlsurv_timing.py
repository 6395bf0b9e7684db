"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan_surv on device rows (one observed scan plus P
permutations in one call) against cnf2_qtl_scan_binary of the status column at the same shape on the same rows, with the mean
iterations per fitted cell of the observed column, the share of the fits by status, and the device's clock.  One process, the
calls alternating, on a synthetic F2 (synth.make_f2): by default 1 000 individuals x 10 chromosomes x 499 SNPs (+1 dummy
marker each) = 5 000 markers, one (time, status) trait with 30 % censored, two covariates, 100 permutations, tol = 1e-7 and
max_iter = 50 for both scans.
usage: python tools/qtlsurv_timing.py [individuals=1000] [snps_per_chrom=499] [chroms=10] [repeats=3] [P=100]"""
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
m1 = M // 3
g = ped.allele[3:, m1, :].astype(np.float64).sum(axis=1) - 3.0
z = np.stack([np.where(synth.uniform(78, np.arange(n)) < 0.5, -0.5, 0.5), synth.uniform(79, np.arange(n)) - 0.5], axis=1)
haz = np.exp(0.5 * g + 0.8 * z[:, 0])
life = -np.log1p(-synth.uniform(77, np.arange(n))) / haz
cens = -np.log1p(-synth.uniform(76, np.arange(n))) / (haz.mean() * 0.3 / 0.7)
t, d = np.minimum(life, cens)[:, None], (life <= cens).astype(np.float64)[:, None]
perm = qtl.permutations(n, P, 3) if P else None
out = {}


def scan_surv():
    out["surv"] = ctx.qtl_scan_surv_device(n, org.data_ptr(), t, d, cov=z, perm=perm, max_iter=50, tol=1e-7)     # (ends in the call's own synchronise)


def scan_binary():
    out["bin"] = ctx.qtl_scan_binary_device(n, org.data_ptr(), d, cov=z, perm=perm, max_iter=50, tol=1e-7)


calls = [("cnf2_qtl_scan_surv", scan_surv), ("cnf2_qtl_scan_binary", scan_binary)]
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
print("%d F2 x %d markers (%d chromosomes), one (time, status) trait (%d events), two covariates, 1 + %d columns, best of %d; times "
      "in s, ending in a synchronise" % (n, M, chroms, int(d.sum()), P, reps))
for name, _ in calls:
    print("  %-22s %.4f (all: %s)" % (name, min(times[name]), " ".join("%.4f" % v for v in times[name])))
for key, name in (("surv", "survival"), ("bin", "binary (of the status)")):
    o = out[key]
    fitted = o["rank"] > 0
    it, st = o["iters"][0][fitted], o["status"][0][fitted]
    print("  %s, observed column: %d of %d markers fitted, mean iterations per cell %.2f, largest %d; status 0 / 1 / 2 at %.4f / %.4f / "
          "%.4f of the fits; peak %.2f at marker %d (planted %d)" % (name, fitted.sum(), M, it.mean(), it.max(), (st == 0).mean(),
                                                                      (st == 1).mean(), (st == 2).mean(), o["lod"][0].max(),
                                                                      int(o["lod"][0].argmax()), m1))
ts, tb = (min(times[name]) for name, _ in calls)
# every fit of t iterations walks the individuals t + 1 times, forward and backward; the permuted columns' counts are not
# reported, so the observed column's mean stands for all of them
fs = out["surv"]["rank"] > 0
passes = float((out["surv"]["iters"][0][fs] + 1).sum()) * (1 + P)
print("  scan_surv / scan_binary %.2f; about %.3g passes x %d individuals in the survival scan: %.3g individual-passes per second" %
      (ts / tb, passes, n, passes * n / ts))
if P:
    print("  5 %% genome-wide threshold of the survival scan %.2f" % qtl.thresholds(out["surv"]["perm_max"])["genome"][0, 0])
ctx.close()
