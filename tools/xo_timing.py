"""Measurement aid: kernel-inclusive wall time of cnf2_sweep_crossovers with sums only (the form a map step uses) against
the plain cnf2_sweep with dosage rows, both with device outputs (CNF2_OUT_DEVICE, torch tensors), on a synthetic F2
(synth.make_f2).  Config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker each).
usage: python tools/xo_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3]"""
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
ll2 = torch.empty_like(ll)
dos = torch.empty((n, M, 3), dtype=torch.float64, device=dev)
xs = torch.empty((M, 6), dtype=torch.float64, device=dev)
cnt = torch.empty(chroms, dtype=torch.int32, device=dev)


def plain():
    ctx.sweep_device(0, n, f.data_ptr(), ll.data_ptr(), dos.data_ptr(), 0)
    ctx.sync()


def xo():
    rc = ctx.L.cnf2_sweep_crossovers(ctx.h, 0, n, C.c_void_p(f.data_ptr()), C.c_void_p(ll2.data_ptr()), None,
                                     C.c_void_p(xs.data_ptr()), C.c_void_p(cnt.data_ptr()), capi.OUT_DEVICE)
    assert rc == 0, ctx.L.cnf2_last_error(ctx.h)
    ctx.sync()


plain()
xo()
tp, tx = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    plain()
    tp.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    xo()
    tx.append(time.perf_counter() - t0)
assert torch.equal(ll, ll2)
print("%d F2 x %d markers (%d chromosomes; input %.1f s): cnf2_sweep with rows %.3f s, cnf2_sweep_crossovers sums only %.3f s"
      " = %.2f x; crossovers per individual %.3f" % (n, M, chroms, gen_s, min(tp), min(tx), min(tx) / min(tp),
                                                    float((xs[:, 0] + xs[:, 3]).sum()) / n))
ctx.close()
