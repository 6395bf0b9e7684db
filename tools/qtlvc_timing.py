"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan_vc at H = 8, 32 and 64 on device descent rows
against cnf2_qtl_scan_hap at H = 8 and 32 on the same rows, individuals and columns, alternating in one process, on a
synthetic F2 (synth.make_f2) as tools/qtlhap_timing.py sets it up: H = 8 gives every cell of a row its own column, H = 32 and 64
deal four and eight such sets out among the individuals.  One trait; P permutations for every P of the list.
Beside the measured ratio the counted work of a (marker, column) cell beyond the product the two scans share: the fixed-effects
scan substitutes through a packed factor, H (H + 1) / 2 multiply-adds; this scan rotates, rank x H, walks the grid, 40 x rank,
and bisects, (QTLVC_REFINE + 3) x rank terms of a division and four multiply-adds each, then rank logarithms.  Per marker and
call the Jacobi iteration: sweeps x (H - 1) rounds x 3 H^2 / 2 rotated element pairs (not timed apart: reasoned from the counts).
usage: python tools/qtlvc_timing.py [individuals=2000] [snps_per_chrom=500] [chroms=20] [repeats=3] [P,P,...=0,100,1000]"""
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
des = qtl.descent_rows(ctx)
truth = ped.allele[3:, M // 3, :].astype(np.float64).sum(axis=1) - 3.0
pheno = (0.5 * truth + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
cols = {8: np.tile(np.arange(8, dtype=np.int32), (n, 1))}
for H in (32, 64):
    cols[H] = (cols[8] + 8 * (np.arange(n)[:, None] % (H // 8))).astype(np.int32)
print("%d F2 x %d markers (%d chromosomes; input %.1f s), one trait, best of %d; times in s, ending in a synchronise" % (n, M, chroms, gen_s, reps))
for P in perms:
    R = 1 + P
    perm = qtl.permutations(n, P, 3) if P else None
    res = qtl.null_residuals(pheno)
    out = {}

    def hap(H):
        def call():
            out["hap", H] = ctx.qtl_scan_hap_device(n, des.data_ptr(), cols[H], H, res, perm=perm, coef=False)
        return call

    def vc(H):
        def call():
            out["vc", H] = ctx.qtl_scan_vc_device(n, des.data_ptr(), cols[H], H, res, perm=perm, blup=False, evals=False)
        return call

    calls = [("cnf2_qtl_scan_hap H = 8", hap(8), ("hap", 8)), ("cnf2_qtl_scan_vc  H = 8", vc(8), ("vc", 8)),
             ("cnf2_qtl_scan_hap H = 32", hap(32), ("hap", 32)), ("cnf2_qtl_scan_vc  H = 32", vc(32), ("vc", 32)),
             ("cnf2_qtl_scan_vc  H = 64", vc(64), ("vc", 64))]
    for _, fn, _ in calls:
        fn()
    times = {name: [] for name, _, _ in calls}
    for _ in range(reps):
        for name, fn, _ in calls:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    best = {key: min(times[name]) for name, _, key in calls}
    print("P = %d (R = %d columns)" % (P, R))
    for name, _, (kind, H) in calls:
        t = times[name]
        base = best.get(("hap", H))
        rank = int(out[kind, H]["rank"].max()) if kind == "vc" else int(out[kind, H]["df"].max())
        cell = H * (H + 1) / 2.0 if kind == "hap" else rank * H + 40.0 * rank + 24 * 5.0 * rank
        print("  %-26s %.4f (all: %s; spread %.2f %%)%s; rank or df at most %d; counted per cell beyond the product %.0f"
              % (name, min(t), " ".join("%.4f" % v for v in t), 100.0 * (max(t) - min(t)) / min(t),
                 " = %.2f x the fixed-effects scan" % (min(t) / base) if kind == "vc" and base else "", rank, cell))
    print("  peak LOD: hap H = 8 %.2f, vc H = 8 %.2f (h %.3f), vc H = 32 %.2f, vc H = 64 %.2f at markers %d %d %d %d; planted %d; rank -1 at %d markers"
          % (out["hap", 8]["lod"].max(), out["vc", 8]["lod"].max(), out["vc", 8]["h"].flat[int(out["vc", 8]["lod"].argmax())],
             out["vc", 32]["lod"].max(), out["vc", 64]["lod"].max(), int(out["hap", 8]["lod"].argmax()), int(out["vc", 8]["lod"].argmax()),
             int(out["vc", 32]["lod"].argmax()), int(out["vc", 64]["lod"].argmax()), M // 3,
             sum(int((out["vc", H]["rank"] < 0).sum()) for H in (8, 32, 64))))
ctx.close()
