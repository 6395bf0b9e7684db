"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan_cof on device rows with Q = 0, 3 and 6
cofactors against cnf2_qtl_scanx (plain: no interactive covariate, no imprinting) on the same rows and against the origin sweep
that makes the rows (cnf2_sweep_origins, device outputs).  One process, the calls alternating, on a synthetic F2
(synth.make_f2); config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker each), one trait, no
covariate, P permutations for every P of the list.  The cofactors sit in the middle of the first Q chromosomes and are left
out within 25 markers of themselves.
usage: python tools/qtlcof_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3] [P,P,...=0,100]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

a = [int(x) for x in sys.argv[1:5]] + [10000, 2500, 20, 3][len(sys.argv[1:5]):]
n, snps, chroms, reps = a
perms = [int(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "0,100").split(",")]
t0 = time.perf_counter()
ped = synth.make_f2(n, snps, chroms, seed=2)
gen_s = time.perf_counter() - t0
ctx = capi.Context(0)
ctx.upload(ped)
M, dev = ped.n_markers, torch.device("cuda", 0)
cs = np.asarray(ped.chromstarts, np.int64)
f = torch.empty((n, chroms, 8), dtype=torch.float64, device=dev)
ll = torch.empty((n, chroms), dtype=torch.float64, device=dev)
org = torch.empty((n, M, 4), dtype=torch.float64, device=dev)
osum = torch.empty((M, 4), dtype=torch.float64, device=dev)
cnt = torch.empty(chroms, dtype=torch.int32, device=dev)


def sweep():
    ctx.sweep_origins_device(0, n, f.data_ptr(), ll.data_ptr(), org.data_ptr(), None, osum.data_ptr(), cnt.data_ptr())
    ctx.sync()


sweep()
mids = [int((cs[c] + cs[c + 1]) // 2) for c in range(min(6, chroms))]
g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
pheno = (sum(0.3 * g(m) for m in mids) + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
print("%d F2 x %d markers (%d chromosomes; input %.1f s), one trait, no covariate, best of %d; times in s, ending in a synchronise" % (
    n, M, chroms, gen_s, reps))
for P in perms:
    perm = qtl.permutations(n, P, 3) if P else None
    res = qtl.null_residuals(pheno)
    out = {}

    def scanx():
        out["x"] = ctx.qtl_scanx_device(n, org.data_ptr(), res, perm=perm)          # (ends in the call's own synchronise)

    def cof_call(Q):
        cof = np.array(mids[:Q], np.int32)
        c = np.searchsorted(cs, cof, side="right") - 1
        excl = (np.maximum(cof - 25, cs[c]).astype(np.int32), np.minimum(cof + 25, cs[c + 1] - 1).astype(np.int32))
        return lambda: out.__setitem__(Q, ctx.qtl_scan_cof_device(n, org.data_ptr(), res, cof, excl=excl, perm=perm))

    calls = [("cnf2_sweep_origins", sweep), ("cnf2_qtl_scanx plain", scanx)] + [
        ("cnf2_qtl_scan_cof Q = %d" % Q, cof_call(Q)) for Q in (0, 3, 6) if Q <= len(mids)]
    for _, fn in calls:
        fn()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    tw, tx = min(times["cnf2_sweep_origins"]), min(times["cnf2_qtl_scanx plain"])
    print("P = %d (R = %d columns)" % (P, 1 + P))
    for name, _ in calls:
        t = min(times[name])
        spread = (max(times[name]) - t) / t
        print("  %-26s %.4f (all: %s; spread %.2f %%)%s" % (name, t, " ".join("%.4f" % v for v in times[name]), 100 * spread,
                                                             "" if "cof" not in name else "  / scanx %.4f, / sweep %.3f" % (t / tx, t / tw)))
    print("  Q = 0 against cnf2_qtl_scanx lod[..., 0]: %.3g; largest conditional LOD with Q = 3: %.2f at marker %d (effects planted at %s)" % (
        np.abs(out[0]["lod"] - out["x"]["lod"][..., 0]).max(), out[3]["lod"].max(), int(np.argmax(out[3]["lod"][0])), mids))
ctx.close()
