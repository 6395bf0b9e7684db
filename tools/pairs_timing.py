"""Measurement aid: wall time, ending in a device synchronise, of one pair sweep (cnf2_sweep_pairs, rows and sums out) beside
cnf2_sweep_origins (rows and sums out) and the plain cnf2_sweep without rows -- as the cross runs it and on all 64 states
(CNF2_ALL_STATES), the form the pair kernel walks --, and of the linked pair scan
(cnf2_qtl_scan2_linked) beside cnf2_qtl_scan2 on the same rows, without permutations and with P of them.  A synthetic F2
(synth.make_f2): n individuals on `chroms` chromosomes of `snps` SNPs (+1 dummy marker each), every `every`-th marker selected;
device outputs and device rows, a warm context.  The calls alternate in one process, `repeats` times, and the best time of
each is reported with all of them; the shader clock (cnf2_clock_probe) is read before and after.
The step count the pair sweep is held against: an anchor walks on average half its chromosome with four vectors where the
sweep walks it twice with one, so a chromosome's S selected markers cost about S - 1 sweeps without rows on top of the
alpha / beta sweep that feeds them.
usage: python tools/pairs_timing.py [individuals=1000] [snps_per_chrom=249] [chroms=20] [every=10] [permutations=100] [repeats=3]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

a = [int(x) for x in sys.argv[1:7]] + [1000, 249, 20, 10, 100, 3][len(sys.argv[1:7]):]
n, snps, chroms, every, P, reps = a
t0 = time.perf_counter()
ped = synth.make_f2(n, snps, chroms, seed=2)
M, dev = ped.n_markers, torch.device("cuda", 0)
sel = qtl.select_every(ped.chromstarts, every)
ctx = capi.Context(0)
ctx.upload(ped)
pairs = ctx.linked_pairs(sel)
NP, L, S = len(pairs), len(sel), len(sel) // chroms
t = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
f, ll, ll2, ll3, ll4 = t(n, chroms, 8), t(n, chroms), t(n, chroms), t(n, chroms), t(n, chroms)
org, bits, osum = t(n, M, 4), t(n, M, 6), t(M, 4)
joint, jsum, cnt = t(n, NP, 16), t(NP, 16), t(chroms, dtype=torch.int32)
print("%d F2 x %d markers on %d chromosomes (input %.1f s); %d selected loci, %d per chromosome, %d pairs on one chromosome of %d; "
      "joint rows %.0f MB; times in s, ending in a synchronise" % (n, M, chroms, time.perf_counter() - t0, L, S, NP, L * (L - 1) // 2,
                                                                     n * NP * 128 / 1e6), flush=True)


def sync():
    ctx.sync()
    torch.cuda.synchronize(dev)


def plain():
    ctx.sweep_device(0, n, f.data_ptr(), ll.data_ptr(), None, capi.NO_DOSAGE)
    sync()


def plain_all_states():
    ctx.sweep_device(0, n, f.data_ptr(), ll4.data_ptr(), None, capi.NO_DOSAGE | capi.ALL_STATES)
    sync()


def origins():
    ctx.sweep_origins_device(0, n, f.data_ptr(), ll2.data_ptr(), org.data_ptr(), bits.data_ptr(), osum.data_ptr(), cnt.data_ptr())
    sync()


def pair_sweep():
    ctx.sweep_pairs_device(0, n, sel, f.data_ptr(), ll3.data_ptr(), joint.data_ptr(), jsum.data_ptr(), cnt.data_ptr())
    sync()


g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
m1, m2 = int(sel[S // 3]), int(sel[2 * S // 3])
pheno = (g(m1) * g(m2) + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
perm = qtl.permutations(n, P, 5) if P else None
out = {}


def scan(linked, pm):
    def call():
        if linked:
            out[linked, pm is not None] = ctx.qtl_scan2_linked_device(n, org.data_ptr(), joint.data_ptr(), sel, pheno, perm=pm)
        else:
            out[linked, pm is not None] = ctx.qtl_scan2_device(n, org.data_ptr(), sel, pheno, perm=pm)
        sync()
    return call


calls = [("cnf2_sweep without rows", plain), ("cnf2_sweep without rows, 64 states", plain_all_states), ("cnf2_sweep_origins with rows", origins), ("cnf2_sweep_pairs with rows", pair_sweep),
         ("cnf2_qtl_scan2, P = 0", scan(False, None)), ("cnf2_qtl_scan2_linked, P = 0", scan(True, None))]
if P:
    calls += [("cnf2_qtl_scan2, P = %d" % P, scan(False, perm)), ("cnf2_qtl_scan2_linked, P = %d" % P, scan(True, perm))]
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
assert torch.equal(ll, ll2) and torch.equal(ll, ll3) and torch.equal(ll, ll4)
best = {k: min(v) for k, v in times.items()}
for name, _ in calls:
    print("  %-32s best %.4f (all: %s)" % (name, best[name], " ".join("%.4f" % v for v in times[name])))
sw, s64, og, pr = (best[k] for k in ("cnf2_sweep without rows", "cnf2_sweep without rows, 64 states", "cnf2_sweep_origins with rows",
                                    "cnf2_sweep_pairs with rows"))
print("  the pair sweep takes %.2f x the origin sweep, %.2f x the sweep without rows as an F2 runs it (the instantiation that keeps equal "
      "states once) and %.2f x the same sweep on all 64 states (CNF2_ALL_STATES), the form the pair kernel walks; the step count says "
      "about %d x the latter (S - 1 = %d anchors a chromosome on top of the alpha / beta sweep)" % (pr / og, pr / sw, pr / s64, S, S - 1))
print("  the pair sweep writes %.0f MB of rows; the sweep in front of it leaves %.0f MB of alpha / beta rows (8 448 B per individual "
      "and marker), which every anchor's wave reads from its own marker on" % (n * NP * 128 / 1e6, n * M * 8448 / 1e6))
for tag in ["P = 0"] + (["P = %d" % P] if P else []):
    a2, b2 = best["cnf2_qtl_scan2, " + tag], best["cnf2_qtl_scan2_linked, " + tag]
    print("  %s: the linked scan takes %.3f x the plain one (%.4f against %.4f)" % (tag, b2 / a2, b2, a2))
print("  shader clock %.0f MHz before, %.0f MHz after" % (clock0, clock1))
lk, pl = out[True, False], out[False, False]
one = np.zeros((L, L), bool)
one[pairs[:, 0], pairs[:, 1]] = True
assert lk["lod_add"].tobytes() == pl["lod_add"].tobytes() and np.isnan(pl["lod_full"][0][one]).all()
j, k = np.unravel_index(np.nanargmax(np.where(one, lk["lod_full"][0] - lk["lod_add"][0], np.nan)), (L, L))
print("  largest lod_int on one chromosome %.2f at markers (%d, %d), planted (%d, %d); class shares of the pair sums' first margin %s"
      % (lk["lod_full"][0, j, k] - lk["lod_add"][0, j, k], sel[j], sel[k], m1, m2,
         " ".join("%.4f" % v for v in (jsum.cpu().numpy().reshape(NP, 4, 4).sum(axis=2).sum(axis=0) / (n * NP)))))
ctx.close()
