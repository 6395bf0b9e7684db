"""Measurement aid: kernel-inclusive wall time of cnf2_sweep_origins (rows and sums out) against the plain cnf2_sweep with
dosage rows and cnf2_sweep_loo (rows and sums out), all with device outputs (CNF2_OUT_DEVICE, torch tensors), alternating in
one process, on a synthetic F2 (synth.make_f2).  Config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1
dummy marker each).
usage: python tools/origins_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3]"""
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
rows = torch.empty((n, M, 10), dtype=torch.float64, device=dev)      # the largest of the three calls' rows; each call's view of it
dos = rows.view(-1)[:n * M * 3]
loo_r, unl_r = rows.view(-1)[:n * M], rows.view(-1)[n * M:2 * n * M]
org_r, bit_r = rows.view(-1)[:n * M * 4], rows.view(-1)[n * M * 4:]
ls = torch.empty(M, dtype=torch.float64, device=dev)
us = torch.empty(M, dtype=torch.float64, device=dev)
osum = torch.empty((M, 4), dtype=torch.float64, device=dev)
cnt = torch.empty(chroms, dtype=torch.int32, device=dev)
ms = {}


def plain():
    ctx.sweep_device(0, n, f.data_ptr(), ll.data_ptr(), dos.data_ptr(), 0)
    ctx.sync()


def loo():
    ctx.sweep_loo_device(0, n, f.data_ptr(), ll2.data_ptr(), loo_r.data_ptr(), unl_r.data_ptr(), ls.data_ptr(), us.data_ptr(),
                         cnt.data_ptr())
    ctx.sync()


def org():
    ctx.sweep_origins_device(0, n, f.data_ptr(), ll3.data_ptr(), org_r.data_ptr(), bit_r.data_ptr(), osum.data_ptr(), cnt.data_ptr())
    ctx.sync()


calls = (("cnf2_sweep with rows", plain), ("cnf2_sweep_loo with rows", loo), ("cnf2_sweep_origins with rows", org))
for _, fn in calls:
    fn()
times = {name: [] for name, _ in calls}
kms = {name: [] for name, _ in calls}
for _ in range(reps):
    for name, fn in calls:
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
        kms[name].append(ctx.last_kernel_ms())
assert torch.equal(ll, ll2) and torch.equal(ll, ll3)
print("%d F2 x %d markers (%d chromosomes; input %.1f s), best of %d:" % (n, M, chroms, gen_s, reps))
for name, _ in calls:
    t = times[name]
    print("  %-30s %.3f s (all: %s; kernels %s ms) = %.2f x the sweep with rows, %.2f x the leave-one-out call"
          % (name, min(t), " ".join("%.3f" % v for v in t), " ".join("%.1f" % v for v in kms[name]),
             min(t) / min(times[calls[0][0]]), min(t) / min(times[calls[1][0]])))
o = osum.cpu().numpy()
print("  expected class shares over all markers: %s (1:1:1:1 in an F2); contributors %s"
      % (" ".join("%.4f" % v for v in o.sum(axis=0) / o.sum()), sorted(set(cnt.cpu().tolist()))))
ctx.close()
