"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan2 on device rows against the origin sweep that
makes the rows (cnf2_sweep_origins, device outputs) and, as the yardstick of the pair kernel's hot path only, against
torch.bmm in f64 of X'[X | Y] over designs X[n][16] materialised beforehand for a slice of the same pairs, scaled to all pairs
(the torch run never enters the product: it forms no design entry from the 32-byte rows, masks nothing, factors nothing and
has no epilogue).  One process, the three alternating, on a synthetic F2 (synth.make_f2); config 2 of BASELINE: 10 000
individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker each); sel = L evenly spaced markers, one trait, P permutations
for every P of the list.
usage: python tools/qtl2_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3] [L=500] [P,P,...=0,100] [slice=128]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

PEAK = 78.6e12          # f64 matrix peak of the MI355X, FLOP/s
a = [int(x) for x in sys.argv[1:6]] + [10000, 2500, 20, 3, 500][len(sys.argv[1:6]):]
n, snps, chroms, reps, L = a
perms = [int(x) for x in (sys.argv[6] if len(sys.argv) > 6 else "0,100").split(",")]
B = int(sys.argv[7]) if len(sys.argv) > 7 else 128
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
sel = np.unique(np.linspace(0, M - 1, L).round().astype(np.int32))
L = len(sel)
sc = np.searchsorted(np.asarray(ped.chromstarts), sel, side="right") - 1
pairs = L * (L - 1) // 2
# a phenotype with a pure interaction of the true genotypes at two selected markers on different chromosomes
m1, m2 = int(sel[L // 5]), int(sel[(3 * L) // 5])
g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
pheno = (0.5 * g(m1) * g(m2) + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
# the bmm's operands: the full designs of B pairs on different chromosomes, X[B][n][16] (1, a1, d1, a2, d2, the four products, zeros)
jj = np.arange(B) % (L // 4)
kk = L - 1 - (np.arange(B) // (L // 4)) - (np.arange(B) % 7)
assert np.all(sc[jj] != sc[kk])
o1, o2 = org[:, torch.from_numpy(sel[jj]).long().to(dev)], org[:, torch.from_numpy(sel[kk]).long().to(dev)]      # [n][B][4]
a1, d1, a2, d2 = o1[:, :, 3] - o1[:, :, 0], o1[:, :, 1] + o1[:, :, 2], o2[:, :, 3] - o2[:, :, 0], o2[:, :, 1] + o2[:, :, 2]
X = torch.zeros((B, n, 16), dtype=torch.float64, device=dev)
for c, v in enumerate((torch.ones_like(a1), a1, d1, a2, d2, a1 * a2, a1 * d2, d1 * a2, d1 * d2)):
    X[:, :, c] = v.T
print("%d F2 x %d markers (%d chromosomes; input %.1f s), %d selected loci = %d pairs (%d on different chromosomes), one trait, "
      "best of %d; times in s, ending in a synchronise" % (n, M, chroms, gen_s, L, pairs, int((sc[:, None] != sc[None, :]).sum()) // 2, reps))
for P in perms:
    R = 1 + P
    perm = qtl.permutations(n, P, 3) if P else None
    res = qtl.null_residuals(pheno)
    Y = torch.from_numpy(np.concatenate([res] + [res[p] for p in (perm if P else [])], axis=1)).to(dev)
    Z = torch.cat([X, Y[None].expand(B, n, R)], dim=2).contiguous()                                   # [B][n][16 + R]
    Xt = X.transpose(1, 2).contiguous()                                                               # [B][16][n]
    out = {}

    def scan():
        out["got"] = ctx.qtl_scan2_device(n, org.data_ptr(), sel, res, perm=perm)      # (ends in the call's own synchronise)

    def bmm():
        out["C"] = torch.bmm(Xt, Z)
        torch.cuda.synchronize()

    calls = (("cnf2_sweep_origins", sweep), ("cnf2_qtl_scan2", scan), ("torch.bmm f64 (slice)", bmm))
    for _, fn in calls:
        fn()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    flop = 2.0 * 16 * (16 + 16 * ((R + 15) // 16)) * n * pairs                # what the matrix instructions of the pair kernel do
    ts, tb, tw = min(times["cnf2_qtl_scan2"]), min(times["torch.bmm f64 (slice)"]), min(times["cnf2_sweep_origins"])
    tball = tb * pairs / B
    print("P = %d (R = %d columns, %.3g FLOP in the pair kernel's matrix instructions)" % (P, R, flop))
    for name, _ in calls:
        print("  %-22s %.4f (all: %s)" % (name, min(times[name]), " ".join("%.4f" % v for v in times[name])))
    print("  scan2: %.2f TFLOP/s = %.3f of the %.1f TFLOP/s f64 matrix peak (whole call over the matrix instructions' FLOP); scan2 / sweep "
          "%.3f; bmm of %d pairs scaled to %d: %.4f s, scan2 / bmm %.2f (bmm's own spread %.4f s on the slice)" % (
              flop / ts / 1e12, flop / ts / PEAK, PEAK / 1e12, ts / tw, B, pairs, tball, ts / tball, max(times["torch.bmm f64 (slice)"]) - tb))
    got = out["got"]
    s = [r for r in qtl.pair_summary(got["lod_add"], got["lod_full"], sel, ped.chromstarts) if r["full"]]
    best = max(s, key=lambda r: r["lod_int"])
    print("  largest lod_int %.2f (lod_full %.2f) at markers %s (planted %d, %d)%s" % (
        best["lod_int"], best["lod_full"], best["full"], m1, m2,
        "; 5 %% thresholds add %.2f full %.2f int %.2f" % tuple(qtl.thresholds2(got["perm_max"])[k][0, 0] for k in ("add", "full", "int")) if P else ""))
    del out["C"], Y, Z, Xt
ctx.close()
