"""Measurement aid: kernel-inclusive wall time of cnf2_sweep_loo (sums out, the rows kept in the context) against the plain
cnf2_sweep with dosage rows and cnf2_sweep_crossovers with sums only, all with device outputs (CNF2_OUT_DEVICE, torch
tensors), alternating in one process, on a synthetic F2 (synth.make_f2).  Config 2 of BASELINE: 10 000 individuals x 20
chromosomes x 2 500 SNPs (+1 dummy marker each).
usage: python tools/loo_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cnf2freq_amd import capi, synth

a = [int(x) for x in sys.argv[1:]] + [10000, 2500, 20, 3][len(sys.argv) - 1:]
n, snps, chroms, reps = a[:4]
t0 = time.perf_counter()
ped = synth.make_f2(n, snps, chroms, seed=2)
gen_s = time.perf_counter() - t0
ctx = capi.Context(0)
ctx.upload(ped)
M, dev = ped.n_markers, torch.device("cuda", 0)
f = torch.empty((n, chroms, 8), dtype=torch.float64, device=dev)
ll = torch.empty((n, chroms), dtype=torch.float64, device=dev)
ll2, ll3 = torch.empty_like(ll), torch.empty_like(ll)
dos = torch.empty((n, M, 3), dtype=torch.float64, device=dev)
xs = torch.empty((M, 6), dtype=torch.float64, device=dev)
ls = torch.empty(M, dtype=torch.float64, device=dev)
us = torch.empty(M, dtype=torch.float64, device=dev)
cnt = torch.empty(chroms, dtype=torch.int32, device=dev)


def plain():
    ctx.sweep_device(0, n, f.data_ptr(), ll.data_ptr(), dos.data_ptr(), 0)
    ctx.sync()


def xo():
    rc = ctx.L.cnf2_sweep_crossovers(ctx.h, 0, n, C.c_void_p(f.data_ptr()), C.c_void_p(ll2.data_ptr()), None,
                                     C.c_void_p(xs.data_ptr()), C.c_void_p(cnt.data_ptr()), capi.OUT_DEVICE)
    assert rc == 0, ctx.L.cnf2_last_error(ctx.h)
    ctx.sync()


def loo():
    ctx.sweep_loo_device(0, n, f.data_ptr(), ll3.data_ptr(), None, None, ls.data_ptr(), us.data_ptr(), cnt.data_ptr())
    ctx.sync()


calls = (("cnf2_sweep with rows", plain), ("cnf2_sweep_crossovers sums only", xo), ("cnf2_sweep_loo", loo))
for _, fn in calls:
    fn()
times = {name: [] for name, _ in calls}
for _ in range(reps):
    for name, fn in calls:
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
assert torch.equal(ll, ll2) and torch.equal(ll, ll3)
print("%d F2 x %d markers (%d chromosomes; input %.1f s), best of %d:" % (n, M, chroms, gen_s, reps))
for name, _ in calls:
    t = times[name]
    print("  %-34s %.3f s (all: %s) = %.2f x the sweep with rows" % (name, min(t), " ".join("%.3f" % v for v in t),
                                                                   min(t) / min(times[calls[0][0]])))
rep_lod = (us - ls) / 2.302585092994046
print("  mean cost per individual and marker %.4f nats; smallest own-position LOD %.1f" % (float(ls.sum()) / n / M, float(rep_lod.min())))
ctx.close()
