"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan_hap at H = 8 and H = 32 on device descent rows
against cnf2_qtl_scan (additive) on device origin rows, on the same individuals and columns, alternating in one process, on a
synthetic F2 (synth.make_f2) -- the model does not care what a column means: H = 8 gives every cell of a row its own column,
H = 32 deals four such sets out among the individuals (four patterns).  One trait; P permutations for every P of the list.
Beside the measured ratio the counted one: per (individual, marker, column) the additive scan's product takes 2 multiply-adds
(a and d are both accumulated) and the founder-haplotype product 8, whatever H; the factorisation adds n H (H + 1) / 2 per
marker once per call and the epilogue H (H + 1) / 2 + H (K + 1) per (marker, column).
usage: python tools/qtlhap_timing.py [individuals=2000] [snps_per_chrom=500] [chroms=20] [repeats=3] [P,P,...=0,100,1000]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

a = [int(x) for x in sys.argv[1:5]] + [2000, 500, 20, 3][len(sys.argv[1:5]):]
n, snps, chroms, reps = a
perms = [int(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "0,100,1000").split(",")]
t0 = time.perf_counter()
ped = synth.make_f2(n, snps, chroms, seed=2)
gen_s = time.perf_counter() - t0
ctx = capi.Context(0)
ctx.upload(ped)
M, dev = ped.n_markers, torch.device("cuda", 0)
org = qtl.origin_rows(ctx)
des = qtl.descent_rows(ctx)
truth = ped.allele[3:, M // 3, :].astype(np.float64).sum(axis=1) - 3.0
pheno = (0.5 * truth + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
cols = {8: np.tile(np.arange(8, dtype=np.int32), (n, 1))}
cols[32] = (cols[8] + 8 * (np.arange(n)[:, None] % 4)).astype(np.int32)
print("%d F2 x %d markers (%d chromosomes; input %.1f s), one trait, best of %d; times in s, ending in a synchronise" % (n, M, chroms, gen_s, reps))
for P in perms:
    R = 1 + P
    perm = qtl.permutations(n, P, 3) if P else None
    res = qtl.null_residuals(pheno)
    out = {}

    def scan():
        out["add"] = ctx.qtl_scan_device(n, org.data_ptr(), res, perm=perm, additive=True)

    def hap(H):
        def call():
            out[H] = ctx.qtl_scan_hap_device(n, des.data_ptr(), cols[H], H, res, perm=perm, coef=False)
        return call

    calls = (("cnf2_qtl_scan additive", scan), ("cnf2_qtl_scan_hap H = 8", hap(8)), ("cnf2_qtl_scan_hap H = 32", hap(32)))
    for _, fn in calls:
        fn()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    ts = min(times[calls[0][0]])
    print("P = %d (R = %d columns)" % (P, R))
    for (name, _), H in zip(calls, (0, 8, 32)):
        t = times[name]
        mac_scan = 2.0 * n * M * R
        mac = mac_scan if H == 0 else 8.0 * n * M * R + n * M * H * (H + 1) / 2.0 + M * R * (H * (H + 1) / 2.0 + H)
        print("  %-26s %.4f (all: %s; spread %.2f %%) = %.2f x the additive scan; counted multiply-adds %.3g = %.2f x"
              % (name, min(t), " ".join("%.4f" % v for v in t), 100.0 * (max(t) - min(t)) / min(t), min(t) / ts, mac, mac / mac_scan))
    print("  peak LOD: additive %.2f at marker %d, H = 8 %.2f (df %d .. %d), H = 32 %.2f (df %d .. %d); planted %d"
          % (out["add"]["lod"].max(), int(out["add"]["lod"].argmax()), out[8]["lod"].max(), out[8]["df"].min(), out[8]["df"].max(),
             out[32]["lod"].max(), out[32]["df"].min(), out[32]["df"].max(), M // 3))
ctx.close()
