"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scanx on device rows -- plain (no interactive
covariate, no imprinting), with imprinting, and with imprinting and one interactive covariate -- against cnf2_qtl_scan on the
same rows and against the origin sweep that makes the rows (cnf2_sweep_origins, device outputs).  One process, the calls
alternating, on a synthetic F2 (synth.make_f2); config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1
dummy marker each), one trait, one covariate, P permutations for every P of the list.
usage: python tools/qtlx_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3] [P,P,...=0,100]"""
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
perms = [int(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "0,100").split(",")]
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
# a phenotype whose additive effect at one marker depends on the covariate
m1 = M // 3
g = ped.allele[3:, m1, :].astype(np.float64).sum(axis=1) - 3.0
z = np.where(synth.uniform(78, np.arange(n)) < 0.5, -0.5, 0.5)[:, None]
pheno = (0.3 * g + 0.6 * g * z[:, 0] + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
print("%d F2 x %d markers (%d chromosomes; input %.1f s), one trait, one covariate, best of %d; times in s, ending in a synchronise" % (
    n, M, chroms, gen_s, reps))
for P in perms:
    R = 1 + P
    perm = qtl.permutations(n, P, 3) if P else None
    res = qtl.null_residuals(pheno, z)
    out = {}
    forms = (("plain", dict(interactive=0, imprint=False), 4), ("imprint", dict(interactive=0, imprint=True), 5),
             ("imprint + 1 interactive", dict(interactive=1, imprint=True), 8))

    def scan():
        out["scan"] = ctx.qtl_scan_device(n, org.data_ptr(), res, cov=z, perm=perm)          # (ends in the call's own synchronise)

    def scanx(kw):
        return lambda: out.__setitem__(kw["imprint"] * 2 + kw["interactive"], ctx.qtl_scanx_device(n, org.data_ptr(), res, cov=z, perm=perm, **kw))

    calls = [("cnf2_sweep_origins", sweep), ("cnf2_qtl_scan", scan)] + [("cnf2_qtl_scanx " + name, scanx(kw)) for name, kw, _ in forms]
    for _, fn in calls:
        fn()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    tw, ts = min(times["cnf2_sweep_origins"]), min(times["cnf2_qtl_scan"])
    print("P = %d (R = %d columns)" % (P, R))
    for name, _ in calls:
        print("  %-38s %.4f (all: %s)" % (name, min(times[name]), " ".join("%.4f" % v for v in times[name])))
    for name, kw, W in forms:
        tx = min(times["cnf2_qtl_scanx " + name])
        # per marker and block of 64 columns: n / 4 k-steps of one 16 x 16 x 4 Gram instruction and four X'Y instructions
        blocks = (R + 63) // 64
        flop = 2.0 * 16 * 16 * 5 * n * M * blocks
        print("  scanx %-24s W = %d: scanx / scan %.2f, scanx / sweep %.3f; %.3g FLOP in the marker kernel's matrix instructions = "
              "%.2f TFLOP/s = %.3f of the %.1f TFLOP/s f64 matrix peak (whole call)" % (name, W, tx / ts, tx / tw, flop, flop / tx / 1e12, flop / tx / PEAK, PEAK / 1e12))
    plain, one = out[0], out["scan"]
    print("  plain lod[..., 0] against cnf2_qtl_scan: %.3g; largest interaction LOD %.2f at marker %d (planted %d)%s" % (
        np.abs(plain["lod"][..., 0] - one["lod"]).max(), (out[3]["lod"][0, :, 2] - out[3]["lod"][0, :, 1]).max(),
        int(np.argmax(out[3]["lod"][0, :, 2] - out[3]["lod"][0, :, 1])), m1,
        "; 5 %% genome-wide threshold of the interaction test %.2f" % qtl.thresholdsx(out[3]["perm_max"])["interaction"]["genome"][0, 0] if P else ""))
ctx.close()
