"""Measurement aid: kernel-inclusive wall time of cnf2_sweep_descent (rows out) against cnf2_sweep_origins (rows and sums
out) of the same tree, both with device outputs (CNF2_OUT_DEVICE, torch tensors), alternating in one process, on a synthetic
F2 (synth.make_f2).  Config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker each).  The
descent call writes 64 bytes a unit against 80 and reduces the same eight values by halving (13 lane exchanges and one store
by eight lanes, against 48 exchanges and ten stores by one lane) and has no finish kernel.
usage: python tools/descent_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3]"""
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
ll2 = torch.empty_like(ll)
rows = torch.empty((n, M, 10), dtype=torch.float64, device=dev)      # the larger of the two calls' rows; each call's view of it
org_r, bit_r = rows.view(-1)[:n * M * 4], rows.view(-1)[n * M * 4:]
des_r = rows.view(-1)[:n * M * 8]
osum = torch.empty((M, 4), dtype=torch.float64, device=dev)
cnt = torch.empty(chroms, dtype=torch.int32, device=dev)


def org():
    ctx.sweep_origins_device(0, n, f.data_ptr(), ll.data_ptr(), org_r.data_ptr(), bit_r.data_ptr(), osum.data_ptr(), cnt.data_ptr())
    ctx.sync()


def des():
    ctx.sweep_descent_device(0, n, f.data_ptr(), ll2.data_ptr(), des_r.data_ptr(), cnt.data_ptr())
    ctx.sync()


calls = (("cnf2_sweep_origins with rows", org), ("cnf2_sweep_descent with rows", des))
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
assert torch.equal(ll, ll2)
print("%d F2 x %d markers (%d chromosomes; input %.1f s), best of %d:" % (n, M, chroms, gen_s, reps))
for name, _ in calls:
    t = times[name]
    print("  %-30s %.3f s (all: %s; spread %.2f %%; kernels %s ms) = %.3f x the origins call"
          % (name, min(t), " ".join("%.3f" % v for v in t), 100.0 * (max(t) - min(t)) / min(t), " ".join("%.1f" % v for v in kms[name]),
             min(t) / min(times[calls[0][0]])))
d = des_r.view(n, M, 8)
print("  each side of a row sums to 1 within %.3g; the strand cells of an F2 differ by at most %.3g"
      % (float((d.view(n, M, 2, 4).sum(dim=3) - 1.0).abs().max()), float((d[:, :, 0::2] - d[:, :, 1::2]).abs().max())))
ctx.close()
